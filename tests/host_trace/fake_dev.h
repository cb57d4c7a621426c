/* fake_dev.h - controls of the recording fake device (fake_dev.c) for driver.c */
#ifndef FAKE_DEV_H
#define FAKE_DEV_H

#include <stdint.h>
#include <stdio.h>

/* forgets every slot / codec state, restarts the call count and arms the fault:
 * the fail_at-th counted call from now returns its failure value (0: none) */
void fake_reset(int fail_at);
/* where the call lines go (NULL: nowhere) */
void fake_trace_to(FILE *f);
/* counted calls since the last reset / whether the armed fault was reached */
int fake_calls(void);
int fake_fault_hit(void);
/* the entry the armed fault failed ("" before it is reached) */
const char *fake_fault_name(void);
/* a failed poll / get_codes: which one since the last qtts_dev_begin, from 1 (other entries: 0) */
int fake_fault_nth(void);
/* FNV-1a over bytes, as the trace prints it */
uint32_t fake_fnv(const void *p, size_t n);

#endif
