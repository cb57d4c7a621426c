/* fake_textfeed.h - controls of the incremental-text fake (fake_textfeed.c) for driver_text_feed.c */
#ifndef FAKE_TEXTFEED_H
#define FAKE_TEXTFEED_H

#include <stdio.h>

/* where its lines go (NULL: nowhere) */
void tf_trace_to(FILE *f);
/* restarts its call count and arms the fault: the fail_at-th text_open / text_append fails (0: none) */
void tf_reset(int fail_at);
int tf_calls(void);
int tf_fault_hit(void);
/* before every generate call: a new run in this length mode (fixed != 0: no EOS) of at most max_frames frames */
void tf_run(int fixed, int max_frames);
/* frames slot b was held in the current run */
int tf_held(int b);

#endif
