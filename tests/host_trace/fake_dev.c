/*
 * fake_dev.c - a recording fake of the device C-ABI (include/qtts_hip.h) for
 * the host trace program: every qtts_dev_* / qtts_hip_* symbol qwen_tts.c
 * references, simulated just far enough for the host's loops to run
 * deterministically on a CPU.
 *
 *   codes   utterance (FNV-1a hash h of its qtts_dev_prompt text ids), frame f,
 *           group g -> code_of(h, f, g); in EOS mode the utterance draws EOS at
 *           frame 3 + h % 9, in fixed mode never
 *   audio   code row r at absolute stream position p -> 1920 samples
 *           sample_of(hash(r), p, j): a wrong frame0, stream or reference cut
 *           gives other samples
 *   trace   one line per call: the entry, its scalars, its arrays in full up
 *           to 8 elements, else length + FNV-1a; no pointers, no times
 *   faults  fake_reset(K): the K-th counted call returns -1 / NULL and does
 *           nothing else (void entries are logged, not counted)
 */
#include "fake_dev.h"

#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/qtts_hip.h"

#define G 16
#define SPF 1920
#define MAXS QTTS_HIP_MAX_BATCH
#define MAX_TAPS 8

struct qtts_dev { qtts_dims_t d; };
struct qtts_codec_snapshot { int pos; };

typedef struct {
    uint32_t pend, hash;         /* the last qtts_dev_prompt's ids / the running utterance's */
    int n_gen, stopped, stop_step, stop_at /* loop step of the EOS */, retired;
    int *codes, *drawn;          /* [max_frames + 1][G] */
    int *force, n_force;         /* [n_force][G] */
} slot_t;

static struct {
    FILE *tr;
    int calls, fail_at, hit;
    const char *hit_name;
    int n_poll, n_get_codes, hit_nth;        /* poll / get_codes calls since the last begin; the failed one's */
    int nb, rows, max_frames, fixed, armed_force, armed_params, n_taps, taps[MAX_TAPS][3];
    slot_t s[MAXS];
    int st_on, st_pos, st_max;               /* the single codec stream */
    int ms_n, ms_max, ms_pos[MAXS];          /* the multi-stream codec (ms_n 0: no begin) */
} F;

/* ------------------------------------------------------------------ helpers */
uint32_t fake_fnv(const void *p, size_t n) {
    const unsigned char *b = (const unsigned char *)p;
    uint32_t h = 2166136261u;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 16777619u;
    return h;
}

static uint32_t mix(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t x = a ^ (b * 2654435761u) ^ (c * 2246822519u);
    x ^= x >> 15; x *= 2654435761u; x ^= x >> 13; x *= 3266489917u; x ^= x >> 16;
    return x;
}

static int code_of(uint32_t h, int f, int g) { return (int)(mix(h, (uint32_t)f, (uint32_t)g) % 2048u); }
static float unit_of(uint32_t x) { return (float)(x & 0xffffu) / 65536.0f - 0.5f; }

static void render(const int *row, int pos, float *out) {
    const uint32_t rh = fake_fnv(row, G * sizeof(int));
    for (int j = 0; j < SPF; j++) out[j] = unit_of(mix(rh, (uint32_t)pos, (uint32_t)j));
}

static void lg(const char *fmt, ...) {
    if (!F.tr) return;
    va_list ap;
    va_start(ap, fmt);
    vfprintf(F.tr, fmt, ap);
    va_end(ap);
}

static void lg_ia(const char *k, const int *a, int n) {
    if (!a) { lg(" %s=NULL", k); return; }
    if (n > 8) { lg(" %s=len %d fnv %08x", k, n, fake_fnv(a, (size_t)n * sizeof(int))); return; }
    lg(" %s=[", k);
    for (int i = 0; i < n; i++) lg(i ? ",%d" : "%d", a[i]);
    lg("]");
}

static void lg_fa(const char *k, const float *a, int n) {
    if (!a) { lg(" %s=NULL", k); return; }
    if (n > 8) { lg(" %s=len %d fnv %08x", k, n, fake_fnv(a, (size_t)n * sizeof(float))); return; }
    lg(" %s=[", k);
    for (int i = 0; i < n; i++) lg(i ? ",%g" : "%g", (double)a[i]);
    lg("]");
}

/* a counted call: 1 when it is the one to fail */
static int enter(const char *name) {
    F.calls++;
    lg("%s", name);
    if (!strcmp(name, "begin")) F.n_poll = F.n_get_codes = 0;
    const int nth = !strcmp(name, "poll") ? ++F.n_poll : !strcmp(name, "get_codes") ? ++F.n_get_codes : 0;
    if (F.calls != F.fail_at) return 0;
    F.hit = 1;
    F.hit_name = name;
    F.hit_nth = nth;
    lg(" -> injected failure\n");
    return 1;
}

static int refuse(const char *why) { lg(" -> refused: %s\n", why); return -1; }

static void slots_free(void) {
    for (int b = 0; b < MAXS; b++) {
        free(F.s[b].codes); free(F.s[b].drawn); free(F.s[b].force);
        memset(&F.s[b], 0, sizeof F.s[b]);
    }
}

void fake_reset(int fail_at) {
    FILE *tr = F.tr;
    slots_free();
    memset(&F, 0, sizeof F);
    F.tr = tr;
    F.fail_at = fail_at;
}

void fake_trace_to(FILE *f) { F.tr = f; }
int fake_calls(void) { return F.calls; }
int fake_fault_hit(void) { return F.hit; }
const char *fake_fault_name(void) { return F.hit_name ? F.hit_name : ""; }
int fake_fault_nth(void) { return F.hit_nth; }

/* ------------------------------------------------------------ device + model */
int qtts_hip_device_count(void) { return 1; }

qtts_dev_t *qtts_dev_create(const qtts_dims_t *dims, int device) {
    if (enter("create")) return NULL;
    lg(" device=%d\n", device);
    qtts_dev_t *dv = (qtts_dev_t *)calloc(1, sizeof *dv);
    if (dv) dv->d = *dims;
    return dv;
}

void qtts_dev_destroy(qtts_dev_t *dv) {
    lg("destroy\n");
    slots_free();
    free(dv);
}

int qtts_dev_put_tensor(qtts_dev_t *dv, const char *name, const void *host, int dtype, const int64_t *shape,
                        int ndim) {
    (void)dv; (void)name; (void)host; (void)dtype; (void)shape; (void)ndim;
    return 0;
}

int qtts_dev_finalize(qtts_dev_t *dv) { (void)dv; return 0; }
size_t qtts_dev_bytes(const qtts_dev_t *dv, int which) { (void)dv; (void)which; return 0; }
int qtts_dev_enc_config(qtts_dev_t *dv, const qtts_enc_dims_t *dims) { (void)dv; (void)dims; return 0; }

int qtts_dev_set_kv_dtype(qtts_dev_t *dv, int dtype) {
    if (enter("set_kv_dtype")) return -1;
    lg(" dtype=%d\n", dtype);
    return dv && (dtype == 0 || dtype == 1) ? 0 : -1;
}

int qtts_dev_kv_dtype(const qtts_dev_t *dv) { return dv ? 0 : -1; }

int qtts_dev_enc_available(qtts_dev_t *dv) {
    if (enter("enc_available")) return -1;
    lg("\n");
    return dv ? 3 : -1;
}

/* --------------------------------------------------------------- generation */
int qtts_dev_begin(qtts_dev_t *dv, int nb, int max_frames, int max_prefill, const qtts_gen_params_t *p) {
    if (enter("begin")) return -1;
    lg(" nb=%d max_frames=%d max_prefill=%d", nb, max_frames, max_prefill);
    if (!dv || !p || nb < 1 || nb > MAXS || max_frames < 1) return refuse("arguments");
    lg(" temperature=%g top_p=%g repetition_penalty=%g top_k=%d st_temperature=%g st_top_p=%g st_top_k=%d"
       " fixed=%d seed=%d\n", (double)p->temperature, (double)p->top_p, (double)p->repetition_penalty, p->top_k,
       (double)p->st_temperature, (double)p->st_top_p, p->st_top_k, p->fixed_codec_tokens, p->seed);
    if (nb != F.nb) F.ms_n = 0;   /* a re-allocation of the state ends the codec streams */
    slots_free();
    F.nb = F.rows = nb;
    F.max_frames = max_frames;
    F.fixed = p->fixed_codec_tokens > 0;
    F.armed_force = F.armed_params = F.n_taps = 0;
    for (int b = 0; b < nb; b++) {
        F.s[b].codes = (int *)calloc((size_t)(max_frames + 1) * G, sizeof(int));
        F.s[b].drawn = (int *)calloc((size_t)(max_frames + 1) * G, sizeof(int));
        F.s[b].stopped = 1;   /* nothing runs in a slot before its prefill */
    }
    return 0;
}

static int slot_bad(const qtts_dev_t *dv, int b) { return !dv || b < 0 || b >= F.nb; }

int qtts_dev_reserve(qtts_dev_t *dv, int max_trailing) {
    if (enter("reserve")) return -1;
    lg(" max_trailing=%d\n", max_trailing);
    return dv && F.nb ? 0 : -1;
}

int qtts_dev_prompt_ref(qtts_dev_t *dv, const int *ref_codes, int n_ref, const float *spk) {
    if (enter("prompt_ref")) return -1;
    lg(" n_ref=%d", n_ref);
    lg_ia("ref_codes", ref_codes, n_ref * G);
    lg_fa("spk", spk, dv ? dv->d.H : 0);
    lg("\n");
    return dv ? 0 : -1;
}

int qtts_dev_prompt(qtts_dev_t *dv, int b, const int *text_ids, int n_text, const int *plan, int nplan, int p_len,
                    int n_trailing, int pad_row) {
    if (enter("prompt")) return -1;
    lg(" b=%d", b);
    lg_ia("text_ids", text_ids, n_text);
    lg_ia("plan", plan, 5 * nplan);
    lg(" p_len=%d n_trailing=%d pad_row=%d\n", p_len, n_trailing, pad_row);
    if (slot_bad(dv, b)) return -1;
    F.s[b].pend = fake_fnv(text_ids, (size_t)n_text * sizeof(int));
    return 0;
}

static void slot_start(int b) {
    slot_t *s = &F.s[b];
    s->hash = s->pend;
    s->n_gen = s->stopped = s->stop_step = s->stop_at = s->retired = 0;
}

int qtts_dev_prefill(qtts_dev_t *dv) {
    if (enter("prefill")) return -1;
    lg("\n");
    if (!dv || !F.nb) return -1;
    for (int b = 0; b < F.nb; b++) slot_start(b);
    return 0;
}

int qtts_dev_refill(qtts_dev_t *dv, int b) {
    if (enter("refill")) return -1;
    lg(" b=%d\n", b);
    if (slot_bad(dv, b) || F.armed_force) return -1;
    slot_start(b);
    return 0;
}

int qtts_dev_retire(qtts_dev_t *dv, int b) {
    if (enter("retire")) return -1;
    lg(" b=%d\n", b);
    if (slot_bad(dv, b)) return -1;
    F.s[b].retired = 1;
    return 0;
}

int qtts_dev_frame(qtts_dev_t *dv, int step) {
    if (enter("frame")) return -1;
    lg(" step=%d\n", step);
    if (!dv || !F.nb) return -1;
    const int eos = dv->d.eos_id;
    for (int b = 0; b < F.rows; b++) {
        slot_t *s = &F.s[b];
        if (s->stopped || s->retired || s->n_gen >= F.max_frames) continue;
        const int f = s->n_gen;
        int *row = s->codes + (size_t)f * G, *dr = s->drawn + (size_t)f * G;
        const int free_eos = !F.fixed && f == 3 + (int)(s->hash % 9u);
        int stop = 0;
        for (int g = 0; g < G; g++) {
            dr[g] = g == 0 && free_eos ? eos : code_of(s->hash, f, g);
            row[g] = dr[g];
            if (f < s->n_force && s->force[(size_t)f * G + g] >= 0) row[g] = s->force[(size_t)f * G + g];
            if (g == 0 && row[0] == eos) {   /* the groups after an EOS are not drawn */
                stop = 1;
                for (int k = 1; k < G; k++) dr[k] = -1;
                break;
            }
        }
        if (stop) {
            s->stopped = 1;
            s->stop_step = f;
            s->stop_at = step;
        } else {
            s->n_gen++;
        }
    }
    return 0;
}

int qtts_dev_poll(qtts_dev_t *dv, int *stopped, int *n_gen, int *stop_step) {
    if (enter("poll")) return -1;
    lg(" stopped=%d n_gen=%d stop_step=%d\n", stopped != NULL, n_gen != NULL, stop_step != NULL);
    if (!dv || !F.nb) return -1;
    for (int b = 0; b < F.nb; b++) {
        if (stopped) stopped[b] = F.s[b].stopped;
        if (n_gen) n_gen[b] = F.s[b].n_gen;
        if (stop_step) stop_step[b] = F.s[b].stop_step;
    }
    return 0;
}

static int stopped_by(int b, int step) { return F.s[b].stopped && F.s[b].stop_at <= step; }

int qtts_dev_frame_done(qtts_dev_t *dv, int step, int *all_stopped) {
    if (enter("frame_done")) return -1;
    lg(" step=%d\n", step);
    if (!dv || !F.nb) return -1;
    int all = 1;
    for (int b = 0; b < F.nb; b++) all &= stopped_by(b, step);
    *all_stopped = all;
    return 0;
}

int qtts_dev_frame_stops(qtts_dev_t *dv, int step, int *stopped) {
    if (enter("frame_stops")) return -1;
    lg(" step=%d\n", step);
    if (!dv || !F.nb) return -1;
    for (int b = 0; b < F.nb; b++) stopped[b] = stopped_by(b, step);
    return 0;
}

int qtts_dev_move_slot(qtts_dev_t *dv, int from, int to) {
    if (enter("move_slot")) return -1;
    lg(" from=%d to=%d\n", from, to);
    if (slot_bad(dv, from) || slot_bad(dv, to) || F.armed_force) return -1;
    const slot_t t = F.s[to];
    F.s[to] = F.s[from];
    F.s[from] = t;
    return 0;
}

int qtts_dev_set_rows(qtts_dev_t *dv, int rows) {
    if (enter("set_rows")) return -1;
    lg(" rows=%d\n", rows);
    if (!dv || rows < 1 || rows > F.nb || F.armed_force) return -1;
    F.rows = rows;
    return 0;
}

int qtts_dev_get_codes(qtts_dev_t *dv, int b, int *host_codes, int max_frames) {
    if (enter("get_codes")) return -1;
    lg(" b=%d max_frames=%d\n", b, max_frames);
    if (slot_bad(dv, b) || max_frames < 0) return -1;
    const int n = F.s[b].n_gen < max_frames ? F.s[b].n_gen : max_frames;
    memcpy(host_codes, F.s[b].codes, (size_t)n * G * sizeof(int));
    return n;
}

/* ------------------------------------------------------ forcing, taps, rows */
int qtts_dev_force(qtts_dev_t *dv, int b, const int *codes, int n_frames) {
    if (enter("force")) return -1;
    lg(" b=%d n_frames=%d", b, n_frames);
    lg_ia("codes", codes, n_frames * G);
    lg("\n");
    if (slot_bad(dv, b) || n_frames < 0 || n_frames > F.max_frames || F.armed_params) return -1;
    slot_t *s = &F.s[b];
    free(s->force);
    s->force = (int *)malloc((size_t)(n_frames > 0 ? n_frames : 1) * G * sizeof(int));
    if (n_frames > 0) memcpy(s->force, codes, (size_t)n_frames * G * sizeof(int));
    s->n_force = n_frames;
    F.armed_force = 1;
    return 0;
}

int qtts_dev_tap(qtts_dev_t *dv, int b, int frame, int group) {
    if (enter("tap")) return -1;
    lg(" b=%d frame=%d group=%d\n", b, frame, group);
    if (slot_bad(dv, b) || F.n_taps >= MAX_TAPS || F.armed_params) return -1;
    F.taps[F.n_taps][0] = b; F.taps[F.n_taps][1] = frame; F.taps[F.n_taps][2] = group;
    F.armed_force = 1;
    return F.n_taps++;
}

int qtts_dev_get_drawn(qtts_dev_t *dv, int b, int *host, int max_frames) {
    if (enter("get_drawn")) return -1;
    lg(" b=%d max_frames=%d\n", b, max_frames);
    if (slot_bad(dv, b) || !F.armed_force) return -1;
    int n = F.s[b].n_gen + F.s[b].stopped;
    if (n > max_frames) n = max_frames;
    memcpy(host, F.s[b].drawn, (size_t)n * G * sizeof(int));
    return n;
}

int qtts_dev_get_tap(qtts_dev_t *dv, int i, float *logits_host, int max_n, unsigned *rng_bits, int *drawn) {
    if (enter("get_tap")) return -1;
    lg(" i=%d max_n=%d\n", i, max_n);
    if (!dv || i < 0 || i >= F.n_taps) return -1;
    const int b = F.taps[i][0], f = F.taps[i][1], g = F.taps[i][2];
    const slot_t *s = &F.s[b];
    if (!(f < s->n_gen || (f == s->n_gen && s->stopped && g == 0))) return -1;
    for (int k = 0; k < 4 && k < max_n && logits_host; k++) logits_host[k] = unit_of(mix(s->hash, (uint32_t)(f * G + g), (uint32_t)k));
    if (rng_bits) *rng_bits = mix(s->hash, (uint32_t)f, 77u + (uint32_t)g);
    if (drawn) *drawn = s->drawn[(size_t)f * G + g];
    return 4;
}

int qtts_dev_slot_params(qtts_dev_t *dv, int b, const qtts_slot_params_t *p) {
    if (enter("slot_params")) return -1;
    lg(" b=%d", b);
    if (slot_bad(dv, b) || !p || F.armed_force) return refuse("arguments");
    lg(" temperature=%g top_p=%g repetition_penalty=%g top_k=%d st_temperature=%g st_top_p=%g st_top_k=%d seed=%d\n",
       (double)p->temperature, (double)p->top_p, (double)p->repetition_penalty, p->top_k, (double)p->st_temperature,
       (double)p->st_top_p, p->st_top_k, p->seed);
    F.armed_params = 1;
    return 0;
}

/* ---------------------------------------------------------- full codec pass */
static float *decode_rows(const int *rows, int T, int *out_samples) {
    float *w = (float *)malloc((size_t)T * SPF * sizeof(float));
    if (!w) return NULL;
    for (int t = 0; t < T; t++) render(rows + (size_t)t * G, t, w + (size_t)t * SPF);
    *out_samples = T * SPF;
    return w;
}

float *qtts_dev_codec_slot(qtts_dev_t *dv, int b, int T, int *out_samples) {
    if (enter("codec_slot")) return NULL;
    lg(" b=%d T=%d\n", b, T);
    if (slot_bad(dv, b) || T < 1 || T > F.s[b].n_gen) return NULL;
    return decode_rows(F.s[b].codes, T, out_samples);
}

float *qtts_dev_codec_decode_host(qtts_dev_t *dv, const int *codes, int T, int *out_samples) {
    if (enter("codec_decode_host")) return NULL;
    lg(" T=%d", T);
    lg_ia("codes", codes, T * G);
    lg("\n");
    if (!dv || !codes || T < 1) return NULL;
    return decode_rows(codes, T, out_samples);
}

int qtts_dev_codec_timing(qtts_dev_t *dv, int on) {
    if (enter("codec_timing")) return -1;
    lg(" on=%d\n", on);
    return dv ? 0 : -1;
}

int qtts_dev_codec_stage_ms(const qtts_dev_t *dv, float *ms) { (void)dv; (void)ms; return -1; }

int qtts_dev_codec_multi(qtts_dev_t *dv, int n, const int *const *host_codes, const int *slot, const int *T,
                         float **audio, int *samples) {
    if (enter("codec_multi")) return -1;
    lg(" n=%d", n);
    lg_ia("T", T, n);
    for (int i = 0; i < n; i++) {
        if (host_codes && host_codes[i]) {
            lg(" job%d:host", i);
            lg_ia("codes", host_codes[i], T[i] * G);
        } else {
            lg(" job%d:slot=%d", i, slot[i]);
        }
    }
    lg("\n");
    int bad = !dv || n < 1;
    for (int i = 0; i < n && !bad; i++) {
        audio[i] = NULL;
        samples[i] = 0;
        bad = T[i] < 1 || (!(host_codes && host_codes[i]) && (slot_bad(dv, slot[i]) || T[i] > F.s[slot[i]].n_gen));
    }
    for (int i = 0; i < n && !bad; i++)
        bad = !(audio[i] = decode_rows(host_codes && host_codes[i] ? host_codes[i] : F.s[slot[i]].codes, T[i],
                                       &samples[i]));
    if (!bad) return 0;
    for (int i = 0; i < n; i++) { free(audio[i]); audio[i] = NULL; samples[i] = 0; }
    return -1;
}

/* ------------------------------------------------- the single codec stream */
int qtts_dev_codec_stream_begin_ex(qtts_dev_t *dv, int max_frames, int chunk_frames) {
    if (enter("codec_stream_begin_ex")) return -1;
    lg(" max_frames=%d chunk_frames=%d\n", max_frames, chunk_frames);
    if (!dv || max_frames < 1) return -1;
    F.st_on = 1;
    F.st_pos = 0;
    F.st_max = max_frames;
    return 0;
}

int qtts_dev_codec_stream_begin(qtts_dev_t *dv, int max_frames) {
    if (enter("codec_stream_begin")) return -1;
    lg(" max_frames=%d\n", max_frames);
    if (!dv || max_frames < 1) return -1;
    F.st_on = 1;
    F.st_pos = 0;
    F.st_max = max_frames;
    return 0;
}

static int stream_push(const int *rows, int T, float *out) {
    if (!F.st_on || T < 1 || F.st_pos + T > F.st_max) return -1;
    for (int t = 0; t < T && out; t++) render(rows + (size_t)t * G, F.st_pos + t, out + (size_t)t * SPF);
    F.st_pos += T;
    return T * SPF;
}

int qtts_dev_codec_stream_prime(qtts_dev_t *dv, const int *codes, int T) {
    if (enter("codec_stream_prime")) return -1;
    lg(" T=%d", T);
    lg_ia("codes", codes, T * G);
    lg("\n");
    if (!dv || !codes) return -1;
    return stream_push(codes, T, NULL) < 0 ? -1 : 0;
}

int qtts_dev_codec_stream_push_slot(qtts_dev_t *dv, int b, int frame0, int T, float *host_out) {
    if (enter("codec_stream_push_slot")) return -1;
    lg(" b=%d frame0=%d T=%d\n", b, frame0, T);
    if (slot_bad(dv, b) || frame0 < 0 || T < 1 || frame0 + T > F.s[b].n_gen || !host_out) return -1;
    return stream_push(F.s[b].codes + (size_t)frame0 * G, T, host_out);
}

int qtts_dev_codec_stream_push_host(qtts_dev_t *dv, const int *codes, int T, float *host_out) {
    if (enter("codec_stream_push_host")) return -1;
    lg(" T=%d", T);
    lg_ia("codes", codes, T * G);
    lg("\n");
    if (!dv || !codes || !host_out) return -1;
    return stream_push(codes, T, host_out);
}

/* ------------------------------------------------- the multi-stream codec */
int qtts_dev_codec_mstream_begin(qtts_dev_t *dv, int n_streams, int max_frames, int chunk_frames) {
    if (enter("codec_mstream_begin")) return -1;
    lg(" n_streams=%d max_frames=%d chunk_frames=%d\n", n_streams, max_frames, chunk_frames);
    if (!dv || n_streams < 1 || n_streams > MAXS || max_frames < 1) return -1;
    F.ms_n = n_streams;
    F.ms_max = max_frames;
    memset(F.ms_pos, 0, sizeof F.ms_pos);
    return 0;
}

/* One push of n streams: stream i takes cnt[i] (NULL: T) frames, from slot
 * slots[i] at f0[i] (NULL: f0u) or from host rows codes[i][ld][G]; same_pos:
 * the refusal of streams at different positions.  Returns the largest count
 * times 1920, or -1 with nothing changed. */
static int ms_push(qtts_dev_t *dv, int n, const int *streams, const int *slots, const int *f0, int f0u,
                   const int *codes, int ld, const int *cnt, int T, int same_pos, float *const *out) {
    if (!dv || !F.ms_n) return refuse("no begin");
    if (n < 1 || n > F.ms_n || !streams || (!slots && !codes)) return refuse("arguments");
    int maxc = 0;
    for (int i = 0; i < n; i++) {
        const int c = cnt ? cnt[i] : T, st = streams[i];
        if (st < 0 || st >= F.ms_n) return refuse("stream out of range");
        for (int k = 0; k < i; k++)
            if (streams[k] == st) return refuse("stream listed twice");
        if (c < 1 || (codes && c > ld)) return refuse("count");
        if (same_pos && F.ms_pos[st] != F.ms_pos[streams[0]]) return refuse("streams at different positions");
        if (F.ms_pos[st] + c > F.ms_max) return refuse("past max_frames");
        if (slots) {
            const int a = f0 ? f0[i] : f0u;
            if (slot_bad(dv, slots[i]) || a < 0 || a + c > F.s[slots[i]].n_gen) return refuse("frames outside the slot");
        }
        if (c > maxc) maxc = c;
    }
    lg("\n");
    for (int i = 0; i < n; i++) {
        const int c = cnt ? cnt[i] : T, st = streams[i];
        const int *rows = slots ? F.s[slots[i]].codes + (size_t)(f0 ? f0[i] : f0u) * G : codes + (size_t)i * ld * G;
        for (int t = 0; t < c && out; t++) render(rows + (size_t)t * G, F.ms_pos[st] + t, out[i] + (size_t)t * SPF);
        F.ms_pos[st] += c;
    }
    return maxc * SPF;
}

static int bounded(int n) { return n < 0 ? 0 : n > MAXS ? MAXS : n; }

int qtts_dev_codec_mstream_push_slots(qtts_dev_t *dv, int n, const int *streams, const int *slots, int frame0, int T,
                                      float *const *host_out) {
    if (enter("codec_mstream_push_slots")) return -1;
    lg(" n=%d frame0=%d T=%d", n, frame0, T);
    lg_ia("streams", streams, bounded(n));
    lg_ia("slots", slots, bounded(n));
    return !slots || !host_out ? refuse("arguments") : ms_push(dv, n, streams, slots, NULL, frame0, NULL, 0, NULL, T, 1, host_out);
}

int qtts_dev_codec_mstream_push_slots_at(qtts_dev_t *dv, int n, const int *streams, const int *slots,
                                         const int *frame0, int T, float *const *host_out) {
    if (enter("codec_mstream_push_slots_at")) return -1;
    lg(" n=%d T=%d", n, T);
    lg_ia("streams", streams, bounded(n));
    lg_ia("slots", slots, bounded(n));
    lg_ia("frame0", frame0, bounded(n));
    return !slots || !frame0 || !host_out ? refuse("arguments") : ms_push(dv, n, streams, slots, frame0, 0, NULL, 0, NULL, T, 0, host_out);
}

int qtts_dev_codec_mstream_push_slots_ragged(qtts_dev_t *dv, int n, const int *streams, const int *slots,
                                             const int *frame0, const int *count, float *const *host_out) {
    if (enter("codec_mstream_push_slots_ragged")) return -1;
    lg(" n=%d", n);
    lg_ia("streams", streams, bounded(n));
    lg_ia("slots", slots, bounded(n));
    lg_ia("frame0", frame0, bounded(n));
    lg_ia("count", count, bounded(n));
    return !slots || !frame0 || !count || !host_out ? refuse("arguments")
                                                    : ms_push(dv, n, streams, slots, frame0, 0, NULL, 0, count, 0, 0, host_out);
}

static int ms_push_host(const char *name, qtts_dev_t *dv, int n, const int *streams, const int *codes,
                        const int *cnt, int ld, int T, int same_pos, float *const *out, int need_out) {
    if (enter(name)) return -1;
    lg(" n=%d ld=%d", n, ld);
    if (cnt) lg_ia("counts", cnt, bounded(n));
    else lg(" T=%d", T);
    lg_ia("streams", streams, bounded(n));
    lg_ia("codes", codes, bounded(n) * (ld > 0 ? ld : 0) * G);
    if (!codes || (need_out && !out)) return refuse("arguments");
    return ms_push(dv, n, streams, NULL, NULL, 0, codes, ld, cnt, T, same_pos, out);
}

int qtts_dev_codec_mstream_push_host(qtts_dev_t *dv, int n, const int *streams, const int *codes, int T,
                                     float *const *host_out) {
    return ms_push_host("codec_mstream_push_host", dv, n, streams, codes, NULL, T, T, 1, host_out, 1);
}

int qtts_dev_codec_mstream_push_host_any(qtts_dev_t *dv, int n, const int *streams, const int *codes, int T,
                                         float *const *host_out) {
    return ms_push_host("codec_mstream_push_host_any", dv, n, streams, codes, NULL, T, T, 0, host_out, 1);
}

int qtts_dev_codec_mstream_push_host_ragged(qtts_dev_t *dv, int n, const int *streams, const int *codes,
                                            const int *counts, int ld_frames, float *const *host_out) {
    if (!counts) { enter("codec_mstream_push_host_ragged"); return refuse("counts NULL"); }
    return ms_push_host("codec_mstream_push_host_ragged", dv, n, streams, codes, counts, ld_frames, 0, 0, host_out, 1);
}

int qtts_dev_codec_mstream_prime(qtts_dev_t *dv, int n, const int *streams, const int *codes, const int *counts,
                                 int ld_frames) {
    if (!counts) { enter("codec_mstream_prime"); return refuse("counts NULL"); }
    return ms_push_host("codec_mstream_prime", dv, n, streams, codes, counts, ld_frames, 0, 0, NULL, 0) < 0 ? -1 : 0;
}

static int ms_bad(const qtts_dev_t *dv, int stream) { return !dv || !F.ms_n || stream < 0 || stream >= F.ms_n; }

int qtts_dev_codec_mstream_reset(qtts_dev_t *dv, int stream) {
    if (enter("codec_mstream_reset")) return -1;
    lg(" stream=%d\n", stream);
    if (ms_bad(dv, stream)) return -1;
    F.ms_pos[stream] = 0;
    return 0;
}

qtts_codec_snapshot_t *qtts_dev_codec_mstream_save(qtts_dev_t *dv, int stream) {
    if (enter("codec_mstream_save")) return NULL;
    lg(" stream=%d pos=%d\n", stream, ms_bad(dv, stream) ? -1 : F.ms_pos[stream]);
    if (ms_bad(dv, stream)) return NULL;
    qtts_codec_snapshot_t *s = (qtts_codec_snapshot_t *)malloc(sizeof *s);
    if (s) s->pos = F.ms_pos[stream];
    return s;
}

int qtts_dev_codec_mstream_restore(qtts_dev_t *dv, int stream, const qtts_codec_snapshot_t *snap) {
    if (enter("codec_mstream_restore")) return -1;
    lg(" stream=%d snapshot_pos=%d\n", stream, snap ? snap->pos : -1);
    if (ms_bad(dv, stream) || !snap || snap->pos > F.ms_max) return -1;
    F.ms_pos[stream] = snap->pos;
    return 0;
}

void qtts_dev_codec_snapshot_free(qtts_codec_snapshot_t *snap) {
    if (snap) lg("codec_snapshot_free pos=%d\n", snap->pos);
    free(snap);
}

int qtts_dev_codec_snapshot_pos(const qtts_codec_snapshot_t *snap) {
    if (enter("codec_snapshot_pos")) return -1;
    lg(" -> %d\n", snap ? snap->pos : -1);
    return snap ? snap->pos : -1;
}

/* ------------------------------------------------------ voice-clone encoders */
int qtts_dev_speaker_embed(qtts_dev_t *dv, int nb, const float *const *wav, const int *n, float *out, float *mel_out) {
    if (enter("speaker_embed")) return -1;
    lg(" nb=%d", nb);
    lg_ia("n", n, bounded(nb));
    for (int b = 0; b < nb && b < 16; b++) lg(" wav%d=%08x", b, fake_fnv(wav[b], (size_t)n[b] * sizeof(float)));
    lg("\n");
    (void)mel_out;
    if (!dv || nb < 1 || nb > 16) return -1;
    for (int b = 0; b < nb; b++) {
        const uint32_t h = fake_fnv(wav[b], (size_t)n[b] * sizeof(float));
        for (int i = 0; i < dv->d.H; i++) out[(size_t)b * dv->d.H + i] = unit_of(mix(h, 1u, (uint32_t)i));
    }
    return 0;
}

int qtts_dev_encode_audio(qtts_dev_t *dv, int nb, const float *const *wav, const int *n, int *codes, int max_frames,
                          int *frames, float *latent) {
    if (enter("encode_audio")) return -1;
    lg(" nb=%d max_frames=%d", nb, max_frames);
    lg_ia("n", n, bounded(nb));
    for (int b = 0; b < nb && b < 16; b++) lg(" wav%d=%08x", b, fake_fnv(wav[b], (size_t)n[b] * sizeof(float)));
    lg("\n");
    (void)latent;
    if (!dv || nb < 1 || nb > 16) return -1;
    memset(codes, 0, (size_t)nb * max_frames * G * sizeof(int));
    for (int b = 0; b < nb; b++) {
        const uint32_t h = fake_fnv(wav[b], (size_t)n[b] * sizeof(float));
        frames[b] = (n[b] + SPF - 1) / SPF;
        if (frames[b] > max_frames) return -1;
        for (int f = 0; f < frames[b]; f++)
            for (int g = 0; g < G; g++) codes[((size_t)b * max_frames + f) * G + g] = code_of(h, f, g);
    }
    return 0;
}

/* ----------------------------------- stage wrappers (no scenario uses them) */
int qtts_dev_talker_prefill_host(qtts_dev_t *dv, const float *embeds, int n, float *hidden_out) {
    (void)dv; (void)embeds; (void)n; (void)hidden_out;
    return -1;
}

int qtts_dev_talker_forward_host(qtts_dev_t *dv, const float *embed, float *logits, float *hidden_out) {
    (void)dv; (void)embed; (void)logits; (void)hidden_out;
    return -1;
}

int qtts_dev_subtalker_host(qtts_dev_t *dv, const float *hidden, int first_code, int *out_codes) {
    (void)dv; (void)hidden; (void)first_code; (void)out_codes;
    return -1;
}
