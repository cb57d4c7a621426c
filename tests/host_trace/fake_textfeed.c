/*
 * fake_textfeed.c - the recording fake of the incremental-text device entries
 * (qtts_dev_text_open / _append), next to the unchanged fake_dev.c.
 *
 * fake_dev.c's frames know no gate: they advance every slot that has not
 * stopped.  This layer keeps the gate's arithmetic itself -- per slot the rows
 * published, the open flag and the frames drawn -- and is linked with
 *   -Wl,--wrap=qtts_dev_prompt,--wrap=qtts_dev_frame,--wrap=qtts_dev_poll,--wrap=qtts_dev_retire
 * so that the host's calls of those four pass through here on their way to
 * fake_dev.c (which still logs and counts them and may inject its fault):
 *   frame   a slot is held when its text is open and n_gen >= rows (else it
 *           advances as in fake_dev.c: EOS at frame 3 + h % 9 unless fixed);
 *           a "gate" line names the held slots
 *   poll    reports this layer's counters
 * fake_dev.c's own slots may run ahead of a held slot; its codes depend on
 * (utterance, frame, group) alone, so every frame the host asks for is there
 * and is the same.
 * Faults: tf_reset(K) makes the K-th text_open / text_append fail.
 */
#include "fake_textfeed.h"

#include <stdarg.h>
#include <string.h>

#include "../../include/qtts_hip.h"
#include "fake_dev.h"

#define MAXS QTTS_HIP_MAX_BATCH

static struct {
    FILE *tr;
    int calls, fail_at, hit;
    int nb, fixed, max_frames, fed;
    uint32_t hash[MAXS];
    int rows[MAXS], open[MAXS], n_gen[MAXS], stopped[MAXS], stop_step[MAXS], retired[MAXS], held[MAXS];
} T;

static void lg(const char *fmt, ...) {
    if (!T.tr) return;
    va_list ap;
    va_start(ap, fmt);
    vfprintf(T.tr, fmt, ap);
    va_end(ap);
}

void tf_trace_to(FILE *f) { T.tr = f; }
void tf_reset(int fail_at) {
    FILE *tr = T.tr;
    memset(&T, 0, sizeof T);
    T.tr = tr;
    T.fail_at = fail_at;
}
int tf_calls(void) { return T.calls; }
int tf_fault_hit(void) { return T.hit; }
int tf_held(int b) { return b >= 0 && b < MAXS ? T.held[b] : -1; }

static int enter(const char *name) {
    T.calls++;
    lg("%s", name);
    if (T.calls != T.fail_at) return 0;
    T.hit = 1;
    lg(" -> injected failure\n");
    return 1;
}

/* ------------------------------------------------------------ the new entries */
int qtts_dev_text_open(qtts_dev_t *dv, int b) {
    if (enter("text_open")) return -1;
    lg(" b=%d\n", b);
    if (!dv || b < 0 || b >= T.nb) return -1;
    T.fed = 1;
    T.open[b] = 1;
    T.rows[b] = 0;
    return 0;
}

int qtts_dev_text_append(qtts_dev_t *dv, int b, const int *ids, int n, int close) {
    if (enter("text_append")) return -1;
    lg(" b=%d n=%d close=%d ids=[", b, n, close);
    for (int i = 0; i < n && i < 8; i++) lg(i ? ",%d" : "%d", ids[i]);
    lg(n > 8 ? ",...]" : "]");
    if (!dv || b < 0 || b >= T.nb || !T.open[b] || n < 0 || (n == 0 && !close)) {
        lg(" -> refused\n");
        return -1;
    }
    T.rows[b] += n + (close ? 1 : 0);
    if (close) T.open[b] = 0;
    lg(" rows=%d\n", T.rows[b]);
    return 0;
}

/* ------------------------------------------- the four calls that pass through */
int __real_qtts_dev_prompt(qtts_dev_t *dv, int b, const int *text_ids, int n_text, const int *plan, int nplan,
                           int p_len, int n_trailing, int pad_row);
int __real_qtts_dev_frame(qtts_dev_t *dv, int step);
int __real_qtts_dev_poll(qtts_dev_t *dv, int *stopped, int *n_gen, int *stop_step);
int __real_qtts_dev_retire(qtts_dev_t *dv, int b);

int __wrap_qtts_dev_prompt(qtts_dev_t *dv, int b, const int *text_ids, int n_text, const int *plan, int nplan,
                           int p_len, int n_trailing, int pad_row) {
    const int rc = __real_qtts_dev_prompt(dv, b, text_ids, n_text, plan, nplan, p_len, n_trailing, pad_row);
    if (rc == 0 && b >= 0 && b < MAXS) {
        T.hash[b] = fake_fnv(text_ids, (size_t)n_text * sizeof(int));
        if (b + 1 > T.nb) T.nb = b + 1;
    }
    return rc;
}

/* before every generate call of the driver: a new run (unfed until a text_open) of this length mode */
void tf_run(int fixed, int max_frames) {
    const int calls = T.calls, fail_at = T.fail_at, hit = T.hit;
    FILE *tr = T.tr;
    memset(&T, 0, sizeof T);
    T.tr = tr; T.calls = calls; T.fail_at = fail_at; T.hit = hit;
    T.fixed = fixed;
    T.max_frames = max_frames;
}

int __wrap_qtts_dev_frame(qtts_dev_t *dv, int step) {
    const int rc = __real_qtts_dev_frame(dv, step);
    if (rc != 0 || !T.fed) return rc;
    int any = 0;
    for (int b = 0; b < T.nb; b++) {
        if (T.stopped[b] || T.retired[b] || T.n_gen[b] >= T.max_frames) continue;
        if (T.open[b] && T.n_gen[b] >= T.rows[b]) {
            lg(any++ ? ",%d" : "gate held=[%d", b);
            T.held[b]++;
            continue;
        }
        if (!T.fixed && T.n_gen[b] == 3 + (int)(T.hash[b] % 9u)) {
            T.stopped[b] = 1;
            T.stop_step[b] = T.n_gen[b];
        } else {
            T.n_gen[b]++;
        }
    }
    if (any) lg("]\n");
    return rc;
}

int __wrap_qtts_dev_poll(qtts_dev_t *dv, int *stopped, int *n_gen, int *stop_step) {
    const int rc = __real_qtts_dev_poll(dv, stopped, n_gen, stop_step);
    if (rc != 0 || !T.fed) return rc;
    for (int b = 0; b < T.nb; b++) {
        if (stopped) stopped[b] = T.stopped[b] || T.retired[b];
        if (n_gen) n_gen[b] = T.n_gen[b];
        if (stop_step) stop_step[b] = T.stop_step[b];
    }
    return rc;
}

int __wrap_qtts_dev_retire(qtts_dev_t *dv, int b) {
    const int rc = __real_qtts_dev_retire(dv, b);
    if (rc == 0 && T.fed && b >= 0 && b < MAXS) T.retired[b] = 1;
    return rc;
}
